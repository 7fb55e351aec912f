"""Tables as ``evaluate_tracks`` leaves them (the thirteen columns of an ``*_analysed.csv`` with its dtypes), written with
``DataFrame.to_csv(index=False)``, for the tests of the typed csv reader and of the marks built on the device; and the
reference both compare with: pandas' read under ``annotate._csv_table``'s dtype, then ``annotate.build_marks``."""
import io

import numpy as np
import pandas as pd

ROW_COLUMNS = ["TRACK_ID", "POSITION_T", "POSITION_X", "POSITION_Y", "WIDTH", "HEIGHT", "DEGREES_ANGLE", "angle_diff",
               "moving", "turn_points", "tp_of_tracks", "travelled_dist", "motility_phenotype"]
#: what annotate_video reads of them, as the typed reader takes it, and as pandas does
FIELDS = [("TRACK_ID", np.uint32), ("POSITION_T", np.int64), ("POSITION_X", np.float64, True), ("POSITION_Y", np.float64, True),
          ("moving", np.int8), ("turn_points", np.int8), ("motility_phenotype", np.float64, True)]
PANDAS_DTYPE = {"TRACK_ID": np.int64, "POSITION_T": np.int64, "POSITION_X": np.float64, "POSITION_Y": np.float64,
                "motility_phenotype": object, "moving": np.int8, "turn_points": np.int8}


def analysed(n, n_frames=300, seed=0, order="track", nan_share=0.05, tracks=None):
    """``n`` rows of ``tracks`` (about n / 40) tracks over ``n_frames`` frames.  ``order``: 'track' (sorted by id, then frame,
    as evaluate_tracks writes), 'shuffled' (rows 0 .. 5 of distinct tracks: get_data sorts) or 'repeat' (shuffled, with the id
    of row 0 again in row 3: get_data keeps the file's order)."""
    rng = np.random.default_rng([seed, n, n_frames])
    tracks = max(8, n // 40) if tracks is None else tracks
    ids = np.sort(rng.choice(np.arange(1, 50 * tracks + 7, dtype=np.int64), tracks, replace=False))
    ids[-1] = 4000000000 + seed                                           # above int32
    track = np.sort(rng.integers(0, tracks, n))
    t = rng.integers(0, n_frames, n).astype(np.int64)
    order_tt = np.lexsort((t, track))
    track, t = track[order_tt], t[order_tt]                               # (the same (id, t) twice happens: file order decides)
    x = np.round(rng.uniform(-20.0, 2000.0, n), rng.integers(0, 14))
    y = rng.uniform(-20.0, 1100.0, n)
    x[rng.random(n) < nan_share] = np.nan
    y[rng.random(n) < nan_share / 2] = np.nan
    phenotype = rng.integers(0, 3, tracks).astype(np.int8)[track]
    tp = rng.uniform(0, 3, n)
    tp[rng.random(n) < 0.5] = np.nan
    df = pd.DataFrame({
        "TRACK_ID": ids[track], "POSITION_T": t, "POSITION_X": x, "POSITION_Y": y, "WIDTH": rng.uniform(2, 9, n),
        "HEIGHT": rng.uniform(9, 30, n), "DEGREES_ANGLE": rng.uniform(0, 180, n), "angle_diff": rng.uniform(-90, 90, n),
        "moving": (rng.random(n) < 0.7).astype(np.int8), "turn_points": (rng.random(n) < 0.2).astype(np.int8),
        "tp_of_tracks": tp, "travelled_dist": rng.uniform(0, 50, n), "motility_phenotype": phenotype})
    if order != "track" and n:
        perm = rng.permutation(n)
        df = df.iloc[perm].reset_index(drop=True)
        if n >= 6:
            # the first rows of six tracks moved to the front
            front = df.drop_duplicates("TRACK_ID").index[:6].to_numpy()
            rest = np.setdiff1d(np.arange(n), front)
            df = df.iloc[np.concatenate([front, rest])].reset_index(drop=True)
            assert df.loc[:5, "TRACK_ID"].is_unique
            if order == "repeat":
                df.loc[3, "TRACK_ID"] = df.loc[0, "TRACK_ID"]
                assert not df.loc[:5, "TRACK_ID"].is_unique
    return df.astype({"TRACK_ID": np.int64, "POSITION_T": np.int64, "moving": np.int8, "turn_points": np.int8, "motility_phenotype": np.int8})


def csv_bytes(df, last_newline=True):
    data = df.to_csv(index=False).encode()
    return data if last_newline else data[:-1]


def pandas_columns(data, names=None):
    """pandas' read of the annotate columns (``names``: of some of them), as ``get_data`` does it, without its sort."""
    dtype = PANDAS_DTYPE if names is None else {k: PANDAS_DTYPE[k] for k in names}
    return pd.read_csv(io.BytesIO(data), sep=",", header=0, usecols=list(dtype), dtype=dtype)


def reference_marks(path, n_frames, select_subtype=None):
    """What annotate_video's host path builds for the csv at ``path``: ``(marks, first)``."""
    from ysmr_amd.annotate import build_marks
    from ysmr_amd.helper_file import get_data
    return build_marks(get_data(path, dtype=PANDAS_DTYPE), n_frames, select_subtype)
