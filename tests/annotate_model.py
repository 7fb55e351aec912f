"""The sequential painter of the annotated video, in numpy: frame by frame, mark by mark in table order, text first and
then the dot, later paint over earlier, pixels outside the frame dropped.  Nothing clever: a loop over marks that assigns
pixels.  ``pack_dib`` turns the painted frames into stored 24-bit DIB frames."""
import numpy as np

MARK_DTYPE = np.dtype([("x", "<i4"), ("y", "<i4"), ("track_id", "<u4"), ("style", "<u4")])

GLYPHS = {
    0: "01110 10001 10011 10101 11001 10001 01110",
    1: "00100 01100 00100 00100 00100 00100 01110",
    2: "01110 10001 00001 00010 00100 01000 11111",
    3: "11111 00010 00100 00010 00001 10001 01110",
    4: "00010 00110 01010 10010 11111 00010 00010",
    5: "11111 10000 11110 00001 00001 10001 01110",
    6: "00110 01000 10000 11110 10001 10001 01110",
    7: "11111 00001 00010 00100 01000 01000 01000",
    8: "01110 10001 10001 01110 10001 10001 01110",
    9: "01110 10001 10001 01111 00001 00010 01100",
}
COLOURS = {0: (0, 255, 0), 1: (15, 165, 253), 2: (255, 255, 255)}       # B, G, R


def to_bgr(frames):
    """u8 [n, H, W] (gray: B = G = R) or [n, H, W, 3] -> a fresh [n, H, W, 3]."""
    frames = np.asarray(frames)
    if frames.ndim == 3:
        return np.repeat(frames[..., None], 3, axis=3)
    return frames.copy()


def paint_frame(image, marks):
    """Paint ``marks`` (MARK_DTYPE records, table order) into ``image`` u8 [H, W, 3] in place."""
    height, width = image.shape[:2]

    def put(px, py, colour):
        if 0 <= px < width and 0 <= py < height:
            image[py, px] = colour

    for m in marks:
        x, y, colour = int(m["x"]), int(m["y"]), COLOURS[int(m["style"])]
        for k, ch in enumerate(str(int(m["track_id"]))):
            for r, bits in enumerate(GLYPHS[int(ch)].split()):
                for c, bit in enumerate(bits):
                    if bit == "1":
                        put(x - 10 + 6 * k + c, y - 16 + r, colour)
        put(x, y, colour)
        if int(m["style"]) == 2:
            for dx, dy in ((-1, 0), (1, 0), (0, -1), (0, 1)):
                put(x + dx, y + dy, colour)
    return image


def paint(frames, marks, first):
    """Frames [n, H, W(, 3)] with the marks ``marks[first[i]:first[i + 1]]`` painted into frame i -> u8 [n, H, W, 3]."""
    out = to_bgr(frames)
    for i in range(out.shape[0]):
        paint_frame(out[i], marks[int(first[i]):int(first[i + 1])])
    return out


def pack_dib(bgr, bottom_up, stride=None, frame_bytes=None, fill=0):
    """u8 [n, H, W, 3] -> u8 [n, frame_bytes]: rows ``stride`` bytes apart (default (3W + 3) & ~3), padding bytes zero,
    the last row first if ``bottom_up``; bytes behind the last row (frame_bytes > stride * H) keep ``fill``."""
    n, height, width = bgr.shape[:3]
    stride = (3 * width + 3) & ~3 if stride is None else stride
    frame_bytes = stride * height if frame_bytes is None else frame_bytes
    out = np.full((n, frame_bytes), fill, np.uint8)
    rows = out[:, :stride * height].reshape(n, height, stride)
    rows[...] = 0
    src = bgr[:, ::-1] if bottom_up else bgr
    rows[:, :, :3 * width] = src.reshape(n, height, 3 * width)
    return out
