"""Streams WITHOUT restart markers for the tests of ``ysmr_mjpeg_decode_batch_sync`` and of its model, built from chosen
coefficients by ``build_stream`` of tests/golden/gen_mjpeg_streams.py (Annex K.3 tables; no Pillow).  Every builder returns
(stream, height, width, sampling) and is cached: the tests share what they build."""
import functools
import importlib.util
import os

import numpy as np

import jpeg_decode_model as dm

HERE = os.path.dirname(os.path.abspath(__file__))


@functools.lru_cache(maxsize=None)
def gen():
    spec = importlib.util.spec_from_file_location("gen_mjpeg_streams", os.path.join(HERE, "golden", "gen_mjpeg_streams.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def _shapes(height, width, sampling):
    lh, lv = dm.LUMA_FACTORS[sampling]
    mx, my = -(-width // (8 * lh)), -(-height // (8 * lv))
    return [(my * lv, mx * lh)] + ([(my, mx)] * 2 if sampling else [])


def entropy_bytes(stream):
    """Bytes of the entropy data as the decoder cuts it: without stuffing, up to EOI."""
    start = stream.index(b"\xff\xda")
    start += 2 + int.from_bytes(stream[start + 2:start + 4], "big")
    return len(stream[start:stream.rindex(b"\xff\xd9")].replace(b"\xff\x00", b"\xff"))


def subsequences(stream, subsequence_bytes):
    return -(-entropy_bytes(stream) // subsequence_bytes)


@functools.lru_cache(maxsize=None)
def noise(height, width, sampling, seed=5, filled=12):
    """Random coefficients in the first ``filled`` zigzag places of every block (a third of them zero), random DC."""
    rng = np.random.default_rng(seed)
    planes = []
    for rows, cols in _shapes(height, width, sampling):
        p = np.zeros((rows, cols, 64), np.int64)
        p[..., :filled] = rng.integers(-40, 41, (rows, cols, filled)) * (rng.random((rows, cols, filled)) > 0.33)
        p[..., 0] = rng.integers(-300, 301, (rows, cols))
        planes.append(p)
    quant = [np.full(64, 2 + c) for c in range(len(planes))]
    return gen().build_stream(height, width, sampling, planes, quant), height, width, sampling


@functools.lru_cache(maxsize=None)
def zeros(block_rows, block_cols):
    """Gray, every coefficient zero: six bits per block (DC category 0, end of block), the same six for ever -- a decoder that
    starts off the code's boundaries stays off them."""
    h, w = 8 * block_rows, 8 * block_cols
    return gen().build_stream(h, w, 0, [np.zeros((block_rows, block_cols, 64), np.int64)], [np.full(64, 3)]), h, w, 0


@functools.lru_cache(maxsize=None)
def dense(block_rows=4, block_cols=6, seed=8):
    """Gray: DC differences of category 11 and, sixteen places apart, coefficients of category 10 -- the longest symbols the
    typical tables have (a 16-bit code and 10 bits behind it), most value bits ones: many 0xFF in the data, each stuffed."""
    rng = np.random.default_rng(seed)
    p = np.zeros((block_rows, block_cols, 64), np.int64)
    p[..., 0] = np.where((np.arange(block_rows * block_cols) & 1).reshape(block_rows, block_cols), 1023, -1024)
    for k in (16, 32, 48):
        p[..., k] = rng.choice([1023, 1022, 1021, 1019, 1015, -1023, 767], (block_rows, block_cols))
    h, w = 8 * block_rows, 8 * block_cols
    return gen().build_stream(h, w, 0, [p], [np.full(64, 1)]), h, w, 0


@functools.lru_cache(maxsize=None)
def dc_wrap(block_rows=3, block_cols=9):
    """Gray: a DC difference of +2047 on every block until the prediction has passed 32767 (block 17: 34799), then back down."""
    n = block_rows * block_cols
    steps = np.where(np.arange(n) < 18, 2047, -2047)
    p = np.zeros((n, 64), np.int64)
    p[:, 0] = np.cumsum(steps)
    p[:, 1] = 3
    assert p[:, 0].max() > 32767
    h, w = 8 * block_rows, 8 * block_cols
    return gen().build_stream(h, w, 0, [p.reshape(block_rows, block_cols, 64)], [np.full(64, 1)]), h, w, 0
