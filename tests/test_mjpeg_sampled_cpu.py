"""The model of ``ysmr_mjpeg_encode_batch`` (tests/jpeg_sampled_model.py) without a GPU: against the 4:4:4 model it
extends, against a plainly written downsample, against Pillow and the decoder's model, and the properties of the Huffman
tables it builds per frame."""
import functools
import io
from fractions import Fraction

import numpy as np
import pytest

import jpeg_decode_model as jdm
import jpeg_model as jm
import jpeg_sampled_model as jsm
from test_mjpeg_cpu import checkerboard, images, saturated

SAMPLINGS = (1, 2, 3)
QUALITIES = (1, 50, 90, 100)


@functools.lru_cache(maxsize=None)
def frames():
    """The frames of test_mjpeg_cpu.py, and flat / noise / saturated / checkerboard at a size that is 1 modulo every MCU."""
    rng = np.random.default_rng(17)
    out = dict(images())
    out.update({"flat17x33": np.full((17, 33, 3), 77, np.uint8), "noise17x33": rng.integers(0, 256, (17, 33, 3), dtype=np.uint8),
                "saturated17x33": saturated(17, 33), "checkerboard17x33": checkerboard(17, 33)})
    for a in out.values():
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def encoded(name, quality, sampling, huffman):
    return jsm.encode_info(frames()[name], quality, sampling, huffman)


NAMES = tuple(frames())


@pytest.mark.parametrize("quality", (50, 90, 100))
@pytest.mark.parametrize("name", tuple(images()))
def test_444_with_the_standard_tables_is_the_444_model(name, quality):
    assert jsm.encode(images()[name], quality, 1, 0) == jm.encode(images()[name], quality)
    assert jsm.encode(images()[name], quality) == jm.encode(images()[name], quality)


def _plain_chroma(bgr, sampling, comp):
    """One chrominance plane of the padded frame, sample by sample."""
    h, v = jsm.FACTORS[sampling]
    height, width = bgr.shape[:2]
    rows, cols = 8 * -(-height // (8 * v)), 8 * -(-width // (8 * h))
    full = jm.ycbcr(bgr)[..., comp]
    out = np.zeros((rows, cols), np.int64)
    for y in range(rows):
        for x in range(cols):
            total = 0
            for dy in range(v):
                for dx in range(h):
                    total += int(full[min(v * y + dy, height - 1), min(h * x + dx, width - 1)])
            if sampling == 1:
                out[y, x] = total
            elif sampling == 2:
                out[y, x] = (total + (0, 1)[x % 2]) // 2
            else:
                out[y, x] = (total + (1, 2)[x % 2]) // 4
    return out


@pytest.mark.parametrize("sampling", SAMPLINGS)
@pytest.mark.parametrize("name", ("noise17x33", "saturated17x33", "scene37x50", "flat8x8"))
def test_the_chroma_planes_are_libjpegs_downsample(name, sampling):
    bgr = frames()[name]
    y, cb, cr = jsm.planes(bgr, sampling)
    h, v = jsm.FACTORS[sampling]
    assert y.shape == (v * cb.shape[0], h * cb.shape[1]) and cb.shape[0] % 8 == 0 and cb.shape[1] % 8 == 0
    assert np.array_equal(cb, _plain_chroma(bgr, sampling, 1)) and np.array_equal(cr, _plain_chroma(bgr, sampling, 2))
    height, width = bgr.shape[:2]
    assert np.array_equal(y[:height, :width], jm.ycbcr(bgr)[..., 0])
    assert (y[height:] == y[height - 1]).all() and (y[:, width:] == y[:, width - 1:width]).all()


def test_the_bias_alternates_along_the_output_row():
    """A frame whose Cb is 101 in even and 102 in odd columns: every pair sums to 203, every square to 406."""
    full = np.zeros((16, 32, 3), np.int64)
    full[..., 0], full[..., 1], full[..., 2] = 128, 101 + (np.arange(32) & 1)[None, :], 128
    original = jm.ycbcr
    jm.ycbcr = lambda bgr: full
    try:
        dummy = np.zeros((16, 32, 3), np.uint8)
        assert jsm.planes(dummy, 2)[1][0].tolist() == [101, 102] * 8           # (203 + 0) >> 1, (203 + 1) >> 1
        assert jsm.planes(dummy, 3)[1][0].tolist() == [101, 102] * 8           # (406 + 1) >> 2, (406 + 2) >> 2
    finally:
        jm.ycbcr = original


def _natural(zigzag):
    out = np.zeros_like(zigzag)
    out[..., jm.ZIGZAG] = zigzag
    return out


@pytest.mark.parametrize("quality", QUALITIES)
@pytest.mark.parametrize("sampling", SAMPLINGS)
@pytest.mark.parametrize("name", NAMES)
def test_pillow_and_the_decoders_model_read_every_stream(name, sampling, quality):
    Image = pytest.importorskip("PIL.Image")
    bgr = frames()[name]
    height, width = bgr.shape[:2]
    parsed = []
    for huffman in (0, 1):
        stream, info = encoded(name, quality, sampling, huffman)
        image = Image.open(io.BytesIO(stream))
        image.load()
        assert image.size == (width, height) and image.mode == "RGB" and image.format == "JPEG", huffman
        pillow = np.asarray(image)[..., ::-1]
        status, mine = jdm.decode(stream, height, width, sampling)
        assert status == 0 and np.array_equal(mine, pillow), huffman
        quant, tables, slots, ri, start = jdm._headers(stream, height, width, sampling)
        coef = jdm._coefficients(stream, height, width, sampling, tables, slots, ri, start)
        for c in range(3):
            assert np.array_equal(coef[c], _natural(info["coefficients"][c])), (huffman, c)
        parsed.append(coef)
    for c in range(3):                                                        # tables change bits, not values
        assert np.array_equal(parsed[0][c], parsed[1][c])


@pytest.mark.parametrize("quality", QUALITIES)
@pytest.mark.parametrize("sampling", SAMPLINGS)
@pytest.mark.parametrize("name", NAMES)
def test_every_built_table_is_a_canonical_code_with_the_all_ones_code_free(name, sampling, quality):
    info = encoded(name, quality, sampling, 1)[1]
    for (bits, vals), counts in zip(info["tables"], info["counts"]):
        assert len(bits) == 16 and sum(bits) == len(vals) >= 1
        assert sorted(vals) == [s for s in range(256) if counts[s]]           # only, and all of, the used symbols
        lengths = {}
        at = 0
        for n in range(1, 17):
            group = vals[at:at + bits[n - 1]]
            assert group == sorted(group)                                     # canonical: by length, then by symbol
            lengths.update({s: n for s in group})
            at += bits[n - 1]
        assert all(1 <= n <= 16 for n in lengths.values())
        assert sum(Fraction(1, 1 << n) for n in lengths.values()) < 1         # strictly: the code of all 1-bits is free
        codes = jm._codes(bits, vals)
        assert all(code != (1 << n) - 1 for code, n in codes.values())
        # a heavier symbol never has the longer code
        order = sorted(lengths, key=lambda s: (counts[s], s))
        assert all(lengths[a] >= lengths[b] for a, b in zip(order, order[1:]))


@pytest.mark.parametrize("quality", QUALITIES)
@pytest.mark.parametrize("sampling", SAMPLINGS)
@pytest.mark.parametrize("name", ("flat17x33", "noise17x33", "saturated17x33", "checkerboard17x33", "flat8x8", "noise23x41",
                                  "saturated16x40"))
def test_the_built_tables_never_make_the_frame_longer(name, sampling, quality):
    standard, s_info = encoded(name, quality, sampling, 0)
    built, b_info = encoded(name, quality, sampling, 1)
    print("{} sampling {} q{}: {} bytes standard, {} built; data bits {} and {}".format(
        name, sampling, quality, len(standard), len(built), s_info["data_bits"], b_info["data_bits"]))
    assert len(built) <= len(standard)


@pytest.mark.parametrize("sampling", SAMPLINGS)
def test_a_flat_frame_has_tables_of_one_symbol(sampling):
    info = encoded("flat17x33", 90, sampling, 1)[1]
    dc_lum, ac_lum, dc_chr, ac_chr = info["tables"]
    assert ac_lum[1] == [0x00] and ac_chr[1] == [0x00]                        # EOB alone
    assert dc_chr[1] == [0] and dc_chr[0] == [1] + [0] * 15                   # gray: every Cb / Cr difference is 0, one 1-bit code
    assert ac_lum[0] == [1] + [0] * 15


@pytest.mark.parametrize("sampling", SAMPLINGS)
def test_noise_at_quality_100_takes_the_rare_paths(sampling):
    stream, info = encoded("noise17x33", 100, sampling, 1)
    counts = info["counts"]
    assert max(s & 15 for s in range(256) if counts[1][s]) >= 8               # large categories
    checker = encoded("checkerboard17x33", 50, sampling, 1)[1]
    assert checker["counts"][1][0xF0] > 0 and 0xF0 in checker["tables"][1][1]  # ZRL is a symbol of the built table
    # a block whose last coefficient is not zero has no EOB: a table may lack it altogether
    full = np.zeros((8, 8, 3), np.uint8)
    yy, xx = np.mgrid[:8, :8]
    full[...] = (128 + 100 * np.cos((2 * yy + 1) * 7 * np.pi / 16) * np.cos((2 * xx + 1) * 7 * np.pi / 16))[..., None].astype(np.uint8)
    one = jsm.encode_info(full, 100, 1, 1)[1]
    assert one["counts"][1][0x00] == 0 and 0x00 not in one["tables"][1][1]
