"""Tables for the tests of the device csv writer (csrc/table_csv.hip): the shapes of ``<name>_selected_data.csv`` and
``<name>_analysed.csv`` with every kind of cell the writer tells apart, rows of all-widest and all-narrowest fields, and what
pandas writes for them."""
import numpy as np
import pandas as pd

#: numpy dtype per column type of include/ysmr_hip.h (YSMR_COL_U32 .. YSMR_COL_F64), and the widest / narrowest value of each
TYPES = (np.uint32, np.int64, np.int32, np.int8, np.float64)
WIDEST = {np.uint32: 4294967295, np.int64: -9223372036854775808, np.int32: -2147483648, np.int8: -128,
          np.float64: -1.2345678901234567e-308}
NARROWEST = {np.uint32: 0, np.int64: 0, np.int32: 0, np.int8: 0, np.float64: np.nan}
WIDTH = {np.uint32: 10, np.int64: 20, np.int32: 11, np.int8: 4, np.float64: 24}

SELECTED = (("index", np.int64), ("TRACK_ID", np.uint32), ("POSITION_T", np.uint32), ("POSITION_X", np.float64),
            ("POSITION_Y", np.float64), ("WIDTH", np.float64), ("HEIGHT", np.float64), ("DEGREES_ANGLE", np.float64))
ANALYSED = (("TRACK_ID", np.uint32), ("POSITION_T", np.uint32), ("POSITION_X", np.float64), ("POSITION_Y", np.float64),
            ("WIDTH", np.float64), ("HEIGHT", np.float64), ("DEGREES_ANGLE", np.float64), ("angle_diff", np.int32),
            ("moving", np.int8), ("turn_points", np.int8), ("tp_of_tracks", np.float64), ("travelled_dist", np.float64),
            ("motility_phenotype", np.int8))


def pandas_bytes(df):
    """What ``save_df_to_csv`` puts into the file."""
    return df.to_csv(index=False).encode("utf-8")


def is_wide(values):
    """The writer's wide cells: finite, non-zero, outside 2^-20 <= |v| < 2^24."""
    a = np.abs(np.asarray(values, np.float64))
    return np.isfinite(a) & (a != 0) & ((a < 2.0 ** -20) | (a >= 2.0 ** 24))


def steady_floats(rng, n):
    """Cells of the steady path: in-range values of many digits and of few, NaN, both zeros, both infinities."""
    v = rng.uniform(-700.0, 700.0, n)
    few = rng.random(n) < 0.3
    v[few] = np.float32(rng.uniform(-90, 90, int(few.sum()))).astype(np.float64)
    kind = rng.integers(0, 40, n)
    for k, special in enumerate((np.nan, 0.0, -0.0, np.inf, -np.inf, 2.0 ** -20, -(2.0 ** 24 - 2.0 ** -29), 0.5, 1e-5, 123456.0)):
        v[kind == k] = special
    return v


def wide_floats(rng, n):
    """Cells of the wide kernel: rounding noise around 1e-14, 1e300-sized values, subnormals, the extremes."""
    v = rng.normal(0, 1e-14, n)
    kind = rng.integers(0, 12, n)
    v[kind == 0] = rng.uniform(1e299, 1e301, int((kind == 0).sum()))
    v[kind == 1] = -rng.uniform(1e24, 1e26, int((kind == 1).sum()))
    for k, special in ((2, 5e-324), (3, -1.7976931348623157e308), (4, 2.2250738585072014e-308), (5, 16777216.0),
                       (6, 1.5e-13), (7, -1.2345678901234567e-308), (8, 2.0 ** -20 * (1 - 2.0 ** -53))):
        v[kind == k] = special
    assert is_wide(v).all()
    return v


def shaped(shape, n, seed, wide="some"):
    """A table of ``n`` rows in one of the two shapes.  ``wide``: 'none', 'first' (one wide cell, in the first row), 'last',
    'some' (one float cell in ten) or 'all' (every float cell)."""
    rng = np.random.default_rng(seed)
    cols = {}
    floats = [name for name, dt in shape if dt is np.float64]
    for name, dt in shape:
        if dt is np.float64:
            v = steady_floats(rng, n)
            if wide == "all":
                v = wide_floats(rng, n)
            elif wide == "some":
                pick = rng.random(n) < 0.1
                v[pick] = wide_floats(rng, int(pick.sum()))
            cols[name] = v
        elif dt is np.int64:
            v = rng.integers(0, 10 ** 7, n, dtype=np.int64)
            v[rng.random(n) < 0.05] = np.iinfo(np.int64).min
            v[rng.random(n) < 0.05] = np.iinfo(np.int64).max
            cols[name] = v
        elif dt is np.uint32:
            v = rng.integers(0, 70000, n).astype(np.uint32)
            v[rng.random(n) < 0.05] = 4294967295
            cols[name] = v
        elif dt is np.int32:
            v = rng.integers(-180, 181, n).astype(np.int32)
            v[rng.random(n) < 0.03] = np.iinfo(np.int32).min
            v[rng.random(n) < 0.03] = np.iinfo(np.int32).max
            cols[name] = v
        else:
            cols[name] = rng.choice(np.array([-128, -1, 0, 1, 2, 127], np.int8), n)
    if n and wide in ("first", "last"):
        cols[floats[-1 if wide == "last" else 0]][0 if wide == "first" else n - 1] = 1e-14
    return pd.DataFrame(cols)


def uniform_rows(dtypes, n, pick):
    """``n`` rows over columns c0, c1, ... of ``dtypes``; row r holds the widest fields where ``pick(r)`` is true, else the
    narrowest."""
    widest = np.array([bool(pick(r)) for r in range(n)], bool)
    return pd.DataFrame({"c{}".format(k): np.where(widest, WIDEST[dt], NARROWEST[dt]).astype(dt) for k, dt in enumerate(dtypes)})
