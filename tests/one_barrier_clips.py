"""Detection sequences for tests/test_gpu_batch_one_barrier.py: what the batch link can get wrong once the ranks and the
row of a frame are written behind the NEXT frame's barrier (csrc/batch_link.h, k_batch, above the frame loop).

Pure numpy, stationary blobs, no filter bank: a track's position is its last measurement, a float32 that converts exactly,
so every way of linking the clip -- k_batch in launches of 64 / 7 / 1 frames, the per-frame link, the host tracker -- must
give EQUAL rows.  ``events`` reads births and deaths per frame off the CPU oracle's rows, and every test asserts with it
that its clip holds the event it is named for before any kernel sees the clip."""
import numpy as np

MAX_GONE = 2.0          # a track unseen in three ageing frames is deregistered in the third
CUTS = (64, 7, 1)       # frames per launch


def _frame(points, seed):
    xy = np.asarray(points, np.float64).reshape(-1, 2)
    assert np.array_equal(xy.astype(np.float32).astype(np.float64), xy), "not float32 values"
    rng = np.random.default_rng(seed)
    info = np.column_stack([rng.uniform(1, 9, len(xy)), rng.uniform(1, 9, len(xy)), rng.uniform(0, 90, len(xy))])
    return xy, info.astype(np.float32).astype(np.float64)


def lattice(n, x0=40.0, y0=40.0, step=24.0, per_row=40):
    """n points, `step` px apart: every blob is nearer to itself than to anything else."""
    return [(x0 + step * (i % per_row), y0 + step * (i // per_row)) for i in range(n)]


def events(oracle, frames, max_gone=MAX_GONE):
    """(births, deaths, live): per frame the ids registered in it, the ids deregistered in it, the live tracks behind it."""
    from link_clips import oracle_rows
    rows, live, _ = oracle_rows(oracle, frames, max_disappeared=max_gone, fps=30.0, use_gsff=False)
    ids = [set() for _ in frames]
    for r in rows:
        ids[r[0]].add(r[1])
    births = [sorted(ids[f] - (ids[f - 1] if f else set())) for f in range(len(frames))]
    deaths = [sorted((ids[f - 1] if f else set()) - ids[f]) for f in range(len(frames))]
    return births, deaths, live


def staggered_deaths_clip(n_tracks, n_frames, first=3, per_frame=3, stride=64, births_at=()):
    """`n_tracks` stationary blobs, all seen in frame 0 (ids = lattice order = seats).  From frame `first` on, `per_frame`
    more blobs go missing for good in EVERY frame -- blobs k, k + stride, k + 2 stride, ...: lanes of different waves -- so
    from frame first + 2 on every frame deregisters `per_frame` tracks, until the supply ends.  ``births_at``: frames that
    show new blobs besides (far to the right), more of them than tracks are missing: more detections than tracks, so the
    frame registers and ages nobody."""
    pts = lattice(n_tracks)
    gone_from = {}
    groups = [[k + j * stride for j in range(per_frame)] for k in range(stride)]
    groups = [g for g in groups if max(g) < n_tracks]
    for k, g in enumerate(groups):
        for i in g:
            gone_from[i] = first + k
    extra, frames = [], []
    for f in range(n_frames):
        if f in births_at:      # (more new blobs than there can be tracks waiting to be deregistered)
            extra = extra + [(1300.0 + 24.0 * (len(extra) + j), 60.0 + 7.0 * f) for j in range(4 * per_frame + 4)]
        shown = [p for i, p in enumerate(pts) if gone_from.get(i, n_frames) > f]
        frames.append(_frame(shown + extra, 300 + f))
    return frames


def wipe_out_clip():
    """40 tracks; no detections from frame 1 on: every track dies in frame 3; frame 4 is empty with an empty table; frame 5
    registers 30 tracks into it; frames 6-8 keep them, 9-12 lose five of them again."""
    a, b = lattice(40), lattice(30, x0=52.0, y0=400.0)
    frames = [a, [], [], [], [], b, b, b, b, b[5:], b[5:], b[5:], b[5:]]
    return [_frame(p, 400 + k) for k, p in enumerate(frames)]


def births_beside_deaths_clip():
    """Twelve tracks.  Blob 0 goes missing from frame 1 (dies in frame 3), frame 4 brings three new blobs: a registration
    right behind a death frame.  Blob 1 goes missing from frame 5; frame 7 registers two more blobs (and ages nobody), so
    blob 1's track dies in frame 8: a death right behind a registration frame."""
    p = lattice(12)
    new_a, new_b = lattice(3, x0=700.0, y0=500.0), lattice(2, x0=900.0, y0=700.0)
    frames = [p, p[1:], p[1:], p[1:], p[1:] + new_a, p[2:] + new_a, p[2:] + new_a, p[2:] + new_a + new_b,
              p[2:] + new_a + new_b, p[2:] + new_a + new_b, p[2:] + new_a + new_b]
    return [_frame(q, 500 + k) for k, q in enumerate(frames)]


def stale_rank_contest_clip():
    """An exact tie for a column in the frame after the lower-id contender's older neighbours died.

    Frame 0 registers, in this order: three `old` blobs (ids 0-2), `far` (3), `lo` (4), 25 bystanders (5-29) -- seats
    as ids.  `far` goes missing at once and dies in frame 3: seat 3 is free.  Frame 4 shows `hi` as well: one detection
    more than tracks, `hi` is registered (id 30) into the lowest free seat, 3 -- the HIGHER id in the LOWER seat.  The
    `old` blobs are missing from frame 5 on and die in frame 7.  In frames 8 and 9 `lo` and `hi` are missing and ONE
    detection `d` appears, at exactly the same squared distance from both.  The claim key of frame 8 is built before
    frame 7's deaths have been taken off the ranks.  Returns (frames, contest frame, lo, hi, d)."""
    d = (1100.0, 8.0)
    lo, hi = (d[0] - 3.0, d[1] + 4.0), (d[0] + 4.0, d[1] - 3.0)
    old = [(200.0, 700.0), (260.0, 700.0), (320.0, 700.0)]
    far = (3400.0, 3000.0)
    by = [(2400.0 + 60.0 * i, 1000.0 + 60.0 * j) for j in range(5) for i in range(5)]
    frames = [old + [far, lo] + by] + [old + [lo] + by] * 3 + [old + [lo] + by + [hi]] + [[lo] + by + [hi]] * 3 + [[d] + by] * 2
    return [_frame(p, 600 + k) for k, p in enumerate(frames)], 8, lo, hi, d


def tie_in_a_registration_frame_clip():
    """`lo` (id 0) and `hi` (id 1) both lose their detections in frame 1 and find `d` at exactly the same squared distance,
    in a frame that also shows five new blobs: more detections than tracks, so the frame takes the exact claim path AND
    registers.  Returns (frames, the frame, lo, hi, d)."""
    d = (1100.0, 8.0)
    lo, hi = (d[0] - 3.0, d[1] + 4.0), (d[0] + 4.0, d[1] - 3.0)
    by = [(2400.0 + 60.0 * i, 1000.0 + 60.0 * j) for j in range(5) for i in range(5)]
    new = lattice(5, x0=300.0, y0=2000.0)
    frames = [[lo, hi] + by, [d] + by + new, [d] + by + new, [d] + by + new]
    return [_frame(p, 700 + k) for k, p in enumerate(frames)], 1, lo, hi, d
