"""A PNG reader for the tests, built on zlib alone: 8-bit RGB, not interlaced, all five row filters."""
import struct
import zlib

import numpy as np


def read_png(path):
    """(rgb u8 [H, W, 3], {chunk type: body of its first occurrence}).  Every chunk's CRC is checked."""
    raw = open(path, "rb").read()
    assert raw[:8] == b"\x89PNG\r\n\x1a\n", "not a PNG signature"
    at, chunks, idat, order = 8, {}, [], []
    while at < len(raw):
        (size,) = struct.unpack(">I", raw[at:at + 4])
        kind, body = raw[at + 4:at + 8], raw[at + 8:at + 8 + size]
        (crc,) = struct.unpack(">I", raw[at + 8 + size:at + 12 + size])
        assert crc == zlib.crc32(kind + body) & 0xFFFFFFFF, "CRC of chunk {}".format(kind)
        order.append(kind)
        if kind == b"IDAT":
            idat.append(body)
        else:
            chunks.setdefault(kind, body)
        at += 12 + size
    assert order[0] == b"IHDR" and order[-1] == b"IEND" and at == len(raw)
    w, h, depth, colour, compression, filt, interlace = struct.unpack(">IIBBBBB", chunks[b"IHDR"])
    assert (depth, colour, compression, filt, interlace) == (8, 2, 0, 0, 0), "only 8-bit RGB, not interlaced"
    data = np.frombuffer(zlib.decompress(b"".join(idat)), np.uint8)
    stride = 3 * w
    assert len(data) == h * (stride + 1)
    rows = data.reshape(h, stride + 1)
    out = np.zeros((h, stride), np.uint8)
    if not rows[:, 0].any():                                       # filter 0 throughout: the rows as they are
        out[:] = rows[:, 1:]
    else:
        prev = np.zeros(stride, np.int64)
        for r in range(h):
            kind, line = int(rows[r, 0]), rows[r, 1:].astype(np.int64)
            cur = np.zeros(stride, np.int64)
            if kind in (0, 2):
                cur = (line + (prev if kind == 2 else 0)) & 255
            else:
                for k in range(stride):
                    a = cur[k - 3] if k >= 3 else 0
                    b, c = prev[k], (prev[k - 3] if k >= 3 else 0)
                    if kind == 1:
                        pred = a
                    elif kind == 3:
                        pred = (a + b) // 2
                    else:
                        assert kind == 4, "row filter {}".format(kind)
                        p = a + b - c
                        pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                        pred = a if pa <= pb and pa <= pc else b if pb <= pc else c
                    cur[k] = (line[k] + pred) & 255
            out[r] = cur
            prev = cur
    chunks["order"] = order
    return out.reshape(h, w, 3), chunks
