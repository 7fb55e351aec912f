#!/usr/bin/env python3
"""Generate tests/golden/tracker_lum_*.npz (run in the BUILD container only): the REFERENCE's own ``ysmr/tracker.py``
(imported the way gen_golden.py imports it) fed three-dimensional centroids (x, y, luminosity) with the GSFF off -- the
combination the reference offers for 'include luminosity in tracking calculation' (with the GSFF on its first update
raises).  Only inputs and outputs are stored; same array names as the other tracker fixtures, ``det`` and ``xy`` with
three columns, plus ``max_disappeared``.

Scenario: pairs of objects of unlike brightness (0.5-0.9 against 1.5-2.2) that cross 0.3-1.2 px apart -- the situation the
third coordinate exists for --, dropout, speckles, free-valued coordinates (GSFF off plus a half-pixel grid gives exact ties).

A fixture is REFUSED (assertion) if
  * two tracks tie in any frame (same nearest detection at the same distance in the 3-D matrix): the reference's argsort is
    not stable, so such a fixture would be ill-defined;
  * the third coordinate decides nothing: the same detections run through the reference in 2-D must give a different track
    table in at least a quarter of the frames.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from gen_golden import import_reference  # noqa: E402


def scenario(rng, n_pairs, n_frames, area, dropout=0.03, speckle=1):
    c = rng.uniform(30, area - 30, (n_pairs, 2))
    ang = rng.uniform(0, np.pi, n_pairs)
    t_cross = rng.integers(10, n_frames - 10, n_pairs)
    speed = rng.uniform(0.2, 0.6, n_pairs)
    off = rng.uniform(0.3, 1.2, n_pairs)
    lum = np.stack([rng.uniform(0.5, 0.9, n_pairs), rng.uniform(1.5, 2.2, n_pairs)], 1)
    frames = []
    for f in range(n_frames):
        d = np.stack([np.cos(ang), np.sin(ang)], 1)
        nrm = np.stack([-d[:, 1], d[:, 0]], 1)
        s = ((f - t_cross) * speed)[:, None]
        a = c + d * s + nrm * off[:, None] / 2
        b = c - d * s - nrm * off[:, None] / 2
        pos = np.vstack([a, b])
        l = np.concatenate([lum[:, 0], lum[:, 1]])
        keep = rng.random(len(pos)) >= dropout
        n_keep = int(keep.sum())
        det = pos[keep] + rng.normal(0, 0.15, (n_keep, 2))
        dl = l[keep] + rng.normal(0, 0.03, n_keep)
        k = rng.integers(0, speckle + 1)
        det = np.vstack([det, rng.uniform(0, area, (k, 2))])
        dl = np.concatenate([dl, rng.uniform(0.4, 2.4, k)])
        # (x and y as a float32 holds them -- what a detector delivers, and what ysmr_tracker_run3 takes; still free-valued)
        det = det.astype(np.float32).astype(np.float64)
        p = rng.permutation(len(det))
        info = np.stack([rng.uniform(1, 7, len(det)), rng.uniform(1, 7, len(det)),
                         rng.uniform(-90, 0, len(det))], 1).astype(np.float32).astype(np.float64)
        frames.append((np.column_stack([det[p], dl[p]]), info))
    return frames


def run_tracker(tracker_mod, frames, fps, max_disappeared, dims):
    from scipy.spatial.distance import cdist
    ct = tracker_mod.CentroidTracker(max_disappeared=max_disappeared, fps=fps, use_gsff=False)
    det_all, info_all, det_off = [], [], [0]
    ids_all, xy_all, info_out, gone_all, off = [], [], [], [], [0]
    claims_all, claim_off, next_id = [], [0], []
    tables = []
    for f, (det3, info) in enumerate(frames):
        det = det3[:, :dims]
        rects = [(tuple(float(v) for v in d), (float(i[0]), float(i[1]), float(i[2]))) for d, i in zip(det, info)]
        col_of = {id(r[1]): c for c, r in enumerate(rects)}
        before = list(ct.objects.keys())
        if dims == 3 and before and len(det):       # (the 2-D run is only compared with: its ties are its own business)
            dm = cdist(np.array(list(ct.objects.values())), det.reshape(-1, dims))
            key = np.stack([dm.argmin(1), dm.min(1)], 1)
            assert len(np.unique(key, axis=0)) == len(key), f"tie in frame {f}: fixture would be ill-defined"
        objs, infos = ct.update(rects)
        ids = list(objs.keys())
        claims = [(row, col_of[id(infos[tid])]) for row, tid in enumerate(before)
                  if tid in infos and id(infos[tid]) in col_of]
        det_all.append(det.reshape(-1, dims)); info_all.append(info.reshape(-1, 3)); det_off.append(det_off[-1] + len(det))
        ids_all.append(np.array(ids, dtype=np.int64))
        xy_all.append(np.array([objs[i] for i in ids], dtype=float).reshape(-1, dims))
        info_out.append(np.array([list(infos[i]) for i in ids], dtype=float).reshape(-1, 3))
        gone_all.append(np.array([ct.disappeared[i] for i in ids], dtype=np.int64))
        off.append(off[-1] + len(ids))
        claims_all.append(np.array(claims, dtype=np.int64).reshape(-1, 2)); claim_off.append(claim_off[-1] + len(claims))
        next_id.append(ct.nextObjectID)
        tables.append({i: tuple(objs[i][:2]) for i in ids})
    out = dict(det=np.concatenate(det_all), det_info=np.concatenate(info_all), det_off=np.array(det_off),
               ids=np.concatenate(ids_all), xy=np.concatenate(xy_all), info=np.concatenate(info_out),
               disappeared=np.concatenate(gone_all), off=np.array(off),
               claims=np.concatenate(claims_all), claim_off=np.array(claim_off), next_id=np.array(next_id),
               fps=np.float64(fps), use_gsff=np.bool_(False), n_min=np.int64(0), n_max=np.int64(30), n_f=np.int64(3),
               max_disappeared=np.float64(max_disappeared))
    return out, tables


def fixture(tracker_mod, name, frames, fps, max_disappeared):
    out, t3 = run_tracker(tracker_mod, frames, fps, max_disappeared, 3)
    _, t2 = run_tracker(tracker_mod, frames, fps, max_disappeared, 2)
    differing = sum(a != b for a, b in zip(t3, t2))
    assert 4 * differing >= len(frames), \
        f"{name}: the third coordinate decides too little ({differing} of {len(frames)} frames differ from the 2-D run)"
    np.savez_compressed(os.path.join(HERE, name), **out)
    print(f"{name}: {len(frames)} frames, {differing} differ from the 2-D run, next id {out['next_id'][-1]}, "
          f"{os.path.getsize(os.path.join(HERE, name))} bytes")


def main():
    _, tracker_mod = import_reference()
    fixture(tracker_mod, "tracker_lum_cross.npz", scenario(np.random.default_rng(7), 60, 80, 600.0), 30.0, 30.0)
    # many births and deaths: speckles in every frame, heavy dropout and a short memory -- registration order (CPython set
    # iteration) and deregistration with three coordinates
    fixture(tracker_mod, "tracker_lum_births.npz",
            scenario(np.random.default_rng(11), 30, 60, 400.0, dropout=0.12, speckle=6), 30.0, 4.0)


if __name__ == "__main__":
    main()
