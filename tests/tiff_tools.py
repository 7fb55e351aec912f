"""A minimal TIFF writer for tests: given strip bodies, tags and byte order it lays out a classic (or, for the refusal test, a
BigTIFF-versioned) file, a page per entry, and can place every strip body at an odd offset.  No Pillow."""
import struct

BYTE, SHORT, LONG = 1, 3, 4
_FORMAT = {BYTE: "B", SHORT: "H", LONG: "I"}


def page(width, height, bodies, rows_per_strip=None, compression=1, photometric=1, samples=1, predictor=1, bits=8, extra=None, drop=()):
    """One page: ``bodies`` are its strips as stored.  ``extra``: {tag: (type, [values])} added or replacing; ``drop``: tags left out."""
    return dict(width=width, height=height, bodies=[bytes(b) for b in bodies], rows_per_strip=rows_per_strip, compression=compression,
                photometric=photometric, samples=samples, predictor=predictor, bits=bits, extra=dict(extra or {}), drop=tuple(drop))


def tiff_bytes(pages, byteorder="<", odd=False, version=42):
    """The file: header, then per page its strip bodies (each beginning at an odd offset if ``odd``), the values that do not fit a
    directory entry, and the directory at an even offset."""
    e = byteorder
    out = bytearray((b"II" if e == "<" else b"MM") + struct.pack(e + "HI", version, 0))
    link = 4                                        # where the offset of the next directory goes
    for p in pages:
        offsets = []
        for body in p["bodies"]:
            if odd and len(out) % 2 == 0:
                out += b"\xA5"
            elif not odd and len(out) % 2:
                out += b"\0"
            offsets.append(len(out))
            out += body
        tags = {256: (LONG, [p["width"]]), 257: (LONG, [p["height"]]), 258: (SHORT, [p["bits"]] * p["samples"]),
                259: (SHORT, [p["compression"]]), 262: (SHORT, [p["photometric"]]), 273: (LONG, offsets),
                277: (SHORT, [p["samples"]]), 279: (LONG, [len(b) for b in p["bodies"]])}
        if p["rows_per_strip"] is not None:
            tags[278] = (LONG, [p["rows_per_strip"]])
        if p["predictor"] != 1:
            tags[317] = (SHORT, [p["predictor"]])
        if p["samples"] > 1:
            tags[284] = (SHORT, [1])
        tags.update(p["extra"])
        for tag in p["drop"]:
            tags.pop(tag, None)
        entries = []
        for tag in sorted(tags):
            kind, values = tags[tag]
            data = struct.pack(e + _FORMAT[kind] * len(values), *values)
            if len(data) > 4:
                if len(out) % 2:
                    out += b"\0"
                where = len(out)
                out += data
                data = struct.pack(e + "I", where)
            entries.append(struct.pack(e + "HHI", tag, kind, len(values)) + data.ljust(4, b"\0"))
        if len(out) % 2:
            out += b"\0"
        out[link:link + 4] = struct.pack(e + "I", len(out))
        out += struct.pack(e + "H", len(entries)) + b"".join(entries)
        link = len(out)
        out += struct.pack(e + "I", 0)
    return bytes(out)


def write_tiff(path, pages, **kw):
    with open(path, "wb") as fh:
        fh.write(tiff_bytes(pages, **kw))
    return str(path)
