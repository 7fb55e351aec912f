"""The row rule of the annotated video's marks (csrc/marks_rule.h: which rows are kept, what a row's mark is, its sort key),
built alone with the host compiler (tests/marks_rule_check.cc) and compared with ``annotate.build_marks`` on hand-picked
values: positions that truncate toward zero, that lie beyond int32 or are not finite, frames at both ends of the video, every
style, every subtype.  The kept rows, stably sorted by the header's key, are ``build_marks``' marks, bytes and all; ``first``
follows from the keys as the device's binary search reads it.  No GPU and no library needed."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pandas as pd
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

XS = [-0.7, -0.0, 0.0, 0.99, 3.999, -3.999, 2147483647.5, 2147483648.0, -2147483648.9, 3e9, -3e9, 1e300, -1e300, 5e-324,
      float("nan"), float("inf"), float("-inf"), 12.5]


def compiler():
    for name in ("c++", "g++", "clang++"):
        if shutil.which(name):
            return shutil.which(name)
    return None


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    cxx = compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("marks_rule") / "marks_rule_check")
    built = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "ysmr_amd", "csrc"),
                            "-I", os.path.join(ROOT, "include"), os.path.join(HERE, "marks_rule_check.cc"), "-o", exe],
                           capture_output=True, text=True)
    assert built.returncode == 0, built.stdout + built.stderr
    return exe


def bits(v):
    return "{:016x}".format(struct.unpack("<Q", struct.pack("<d", v))[0])


def table():
    """Every x against a good y and the other way round, over frames -1 .. n_frames; then every style and phenotype."""
    rows = []
    for k, v in enumerate(XS):
        rows.append((v, 7.9, k % 5, 100 + k, 1, 0, 1.0))
        rows.append((-7.9, v, (k + 2) % 5, 200 + k, 1, 0, 2.0))
    for t in (-1, 0, 4, 5, 6, 2 ** 31, 2 ** 40, -2 ** 40):
        rows.append((1.5, 2.5, t, 300, 1, 0, 0.0))
    for moving in (0, 1, -1, 2):
        for turn in (0, 1, -1, 2):
            rows.append((10.0, 20.0, 3, 4000000000 + 4 * moving + turn, moving, turn, 1.0))
    for phenotype in (0.0, 1.0, 2.0, 3.0, 0.5, float("nan")):
        rows.append((30.0, 40.0, 2, 7, 1, 1, phenotype))
    rows.append((1.0, 1.0, 2, 7, 1, 0, 1.0))          # the same (id, t) once more: file order decides
    x, y, t, ids, moving, turn, phenotype = zip(*rows)
    return pd.DataFrame({"TRACK_ID": np.array(ids, np.int64), "POSITION_T": np.array(t, np.int64), "POSITION_X": np.array(x, np.float64),
                         "POSITION_Y": np.array(y, np.float64), "moving": np.array(moving, np.int8),
                         "turn_points": np.array(turn, np.int8), "motility_phenotype": np.array(phenotype, np.float64)})


def run(checker, df, n_frames, subtype, by_track):
    from ysmr_amd import _lib
    text = "".join("{} {} {} {} {} {} {}\n".format(bits(r.POSITION_X), bits(r.POSITION_Y), r.POSITION_T, r.TRACK_ID & 0xFFFFFFFF, r.moving,
                                                   r.turn_points, bits(r.motility_phenotype)) for r in df.itertuples())
    done = subprocess.run([checker, str(n_frames), str(-1 if subtype is None else subtype), str(int(by_track))], input=text,
                          capture_output=True, text=True, timeout=60)
    assert done.returncode == 0, done.stdout + done.stderr
    lines = done.stdout.split("\n")
    assert len(lines) == len(df) + 2
    kept = np.array([int(l.split()[0]) for l in lines[:len(df)]], bool)
    keys = np.array([int(l.split()[1], 16) for l in lines[:len(df)]], np.uint64)
    marks = np.zeros(len(df), _lib.MARK_DTYPE)
    for k, l in enumerate(lines[:len(df)]):
        marks[k] = tuple(int(v) for v in l.split()[2:])
    tail = lines[len(df)].split()
    return kept, keys, marks, int(tail[1]), int(tail[3])


@pytest.mark.parametrize("subtype", [None, 0, 1, 2])
@pytest.mark.parametrize("by_track", [False, True])
def test_kept_rows_sorted_by_the_key_are_build_marks_marks(checker, subtype, by_track):
    from ysmr_amd.annotate import build_marks
    df, n_frames = table(), 5
    kept, keys, marks, key_bits, _distinct = run(checker, df, n_frames, subtype, by_track)
    ordered = df.sort_values(by=["TRACK_ID", "POSITION_T"], kind="stable").reset_index(drop=True) if by_track else df
    want, first = build_marks(ordered, n_frames, subtype)
    assert (keys[~kept] == np.uint64(2 ** 64 - 1)).all() and kept.sum() == len(want) > 0
    assert key_bits == 40 and (keys[kept] < np.uint64(1) << np.uint64(key_bits)).all()
    order = np.argsort(keys, kind="stable")[:kept.sum()]
    got = marks[order]
    assert got.tobytes() == want.tobytes(), [(a, b) for a, b in zip(got, want) if a != b][:5]
    sorted_keys = keys[np.argsort(keys, kind="stable")]
    bounds = np.arange(n_frames + 1, dtype=np.uint64) << np.uint64(32)
    assert np.array_equal(np.searchsorted(sorted_keys, bounds, side="left").astype(np.int64), first)


def test_hand_picked_values(checker):
    df = table()
    kept, _keys, marks, _bits, distinct = run(checker, df, 5, None, False)
    by_x = {bits(x): (k, m) for x, k, m in zip(df["POSITION_X"][:2 * len(XS):2], kept[:2 * len(XS):2], marks[:2 * len(XS):2])}
    for x, want in ((-0.7, 0), (-0.0, 0), (0.99, 0), (3.999, 3), (-3.999, -3), (2147483647.5, 2147483647), (2147483648.0, 2147483647),
                    (-2147483648.9, -2147483648), (3e9, 2147483647), (-3e9, -2147483648), (1e300, 2147483647), (-1e300, -2147483648)):
        assert by_x[bits(x)][0] and by_x[bits(x)][1]["x"] == want, x
    for x in (float("nan"), float("inf"), float("-inf")):
        assert not by_x[bits(x)][0], x
    t_rows = df.index[(df["TRACK_ID"] == 300)]          # t = -1, 0, 4, 5 (= n_frames), 6, 2^31, 2^40, -2^40
    assert [bool(kept[k]) for k in t_rows] == [False, True, True, False, False, False, False, False]
    styles = {(int(r.moving), int(r.turn_points)): int(marks[r.Index]["style"]) for r in df.itertuples() if r.TRACK_ID >= 4000000000 - 8}
    assert styles == {(m, t): (1 if m == 0 else 2 if t == 1 else 0) for m in (0, 1, -1, 2) for t in (0, 1, -1, 2)}
    assert marks[df.index[df["TRACK_ID"] == 4000000001][0]]["track_id"] == 4000000001
    assert distinct == 1


@pytest.mark.parametrize("n_frames,want", [(1, 40), (255, 40), (256, 48), (65535, 48), (65536, 56), (2 ** 24, 64), (2 ** 31 - 2, 64)])
def test_the_sorted_bits_hold_n_frames_itself(checker, n_frames, want):
    df = table().iloc[:3]
    assert run(checker, df, n_frames, None, True)[3] == want


@pytest.mark.parametrize("ids,want", [([1, 2, 3, 4, 5, 6, 1], 1), ([1, 2, 3, 4, 5, 1, 7], 0), ([3, 3], 0), ([3], 1), ([1, 2, 3, 4, 5], 1)])
def test_the_rough_check_looks_at_six_rows_or_all_of_fewer(checker, ids, want):
    df = table().iloc[:len(ids)].copy()
    df["TRACK_ID"] = np.array(ids, np.int64)
    assert run(checker, df, 5, None, True)[4] == want
    assert bool(df.loc[:5, "TRACK_ID"].is_unique) == bool(want)
