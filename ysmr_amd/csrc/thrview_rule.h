// thrview_rule.h -- what the threshold view of track_bacteria ('hip save threshold video') stores for a pixel, in the one form
// that the kernel of thrview.hip, its host twin ysmr_thrview_batch_host and a stand-alone host program all compile (plain
// C++ as well as HIP).
//
// PIXEL RULE.  Of a pixel the view knows its class byte (bit 0: passed the low threshold, "thresh"; bit 1: passed the high
// one, "marker"; other bits are not looked at), the byte of the final mask (not 0: kept by the hysteresis) and, in mode 2,
// the frame's own pixel.  Stored are B, G, R:
//   mode 0  mask     255, 255, 255 where mask != 0, else 0, 0, 0                  (upstream's window 'threshold')
//   mode 1  markers  255, 255, 255 where bit 1 is set, else 0, 0, 0               (... 'Adaptive double threshold markers')
//   mode 2  classes  the first of these that holds, a function of (cls & 3, mask != 0) alone:
//             mask != 0 and bit 1 set      (0, 0, 255)      kept, a marker
//             mask != 0, bit 1 clear       (0, 255, 255)    kept, not a marker
//             mask == 0 and bit 0 set      (255, 0, 0)      passed the low threshold, dropped by the hysteresis
//             otherwise                    the frame's pixel: gray g -> (g, g, g), B, G, R as they are
// The rule is total: combinations no detector produces (a kept pixel without bit 0, a marker that was not kept) have their
// line above like any other.  The frames are stored as DIB frames, as view_rule.h's: rows `stride` bytes apart, the bytes
// behind a row's pixels zero, the last row first if bottom_up, bytes between two frames untouched.
//
// TWO FORMS of the rule, both used by the kernel and by the host loop at the same places of a row: `pixel` for one pixel (a
// row's tail), and `step16` for 16 pixels at once, which works on four pixels per 32-bit word -- a byte of a word is 0xFF or 0
// for "kept", "marker", "thresh", the colours are ANDs of those, and byte selects (v_perm_b32 on the device) lay B, G, R out.
// Byte k of a word is pixel k (little endian, as the device is).
#pragma once
#include <cstddef>
#include <cstdint>
#include "hd.h"
#include "view_rule.h"

namespace ysmr {
namespace thrview {

constexpr int MODE_MASK = 0, MODE_MARKERS = 1, MODE_CLASSES = 2;
constexpr int PAINT_NONE = 0, PAINT_MARKER = 1, PAINT_KEPT = 2, PAINT_DROPPED = 3;

// which of mode 2's lines holds for a pixel
YSMR_HD_FORCE int paint_of(uint32_t cls, uint32_t mask)
{
    if (mask) return (cls & 2u) ? PAINT_MARKER : PAINT_KEPT;
    return (cls & 1u) ? PAINT_DROPPED : PAINT_NONE;
}

// One pixel into p[0 .. 2].  b, g, r: the frame's pixel (looked at in mode 2 only).
YSMR_HD_FORCE void pixel(int mode, uint32_t cls, uint32_t mask, uint8_t b, uint8_t g, uint8_t r, uint8_t *p)
{
    if (mode != MODE_CLASSES) {
        p[0] = p[1] = p[2] = (mode == MODE_MASK ? mask != 0u : (cls & 2u) != 0u) ? 255 : 0;
        return;
    }
    const int paint = paint_of(cls, mask);
    p[0] = paint == PAINT_NONE ? b : paint == PAINT_DROPPED ? 255 : 0;
    p[1] = paint == PAINT_NONE ? g : paint == PAINT_KEPT ? 255 : 0;
    p[2] = paint == PAINT_NONE ? r : paint == PAINT_DROPPED ? 0 : 255;
}

// Byte i of the result is byte sel.byte[i] of the eight bytes b (0 .. 3), a (4 .. 7): v_perm_b32 for selectors 0 .. 7.
YSMR_HD_FORCE uint32_t perm(uint32_t a, uint32_t b, uint32_t sel)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_perm(a, b, sel);
#else
    const uint64_t both = ((uint64_t)a << 32) | b;
    uint32_t out = 0;
    for (int i = 0; i < 4; ++i) out |= (uint32_t)((both >> (8 * ((sel >> (8 * i)) & 7u))) & 0xFFu) << (8 * i);
    return out;
#endif
}

// per byte: 0xFF where the byte is not zero / where its bit `bit` is set, else 0
YSMR_HD_FORCE uint32_t bytes_nonzero(uint32_t w)
{
    return (((((w & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | w) & 0x80808080u) >> 7) * 0xFFu;     // (no carry leaves a byte: 0x7F + 0x7F = 0xFE)
}
YSMR_HD_FORCE uint32_t bytes_bit(uint32_t w, int bit) { return ((w >> bit) & 0x01010101u) * 0xFFu; }

// the four bytes p0 p1 p2 p3 of w, each three times: p0 p0 p0 p1 | p1 p1 p2 p2 | p2 p3 p3 p3
YSMR_HD_FORCE void thrice(uint32_t w, uint32_t *d)
{
    d[0] = perm(w, w, 0x01000000u);
    d[1] = perm(w, w, 0x02020101u);
    d[2] = perm(w, w, 0x03030302u);
}

// Four pixels: c, m their class and mask bytes, fr[0 .. 2] their twelve frame bytes B G R B G R ... (mode 2 only) -> d[0 .. 2].
YSMR_HD_FORCE void quad(int mode, uint32_t c, uint32_t m, const uint32_t *fr, uint32_t *d)
{
    if (mode != MODE_CLASSES) {
        thrice(mode == MODE_MASK ? bytes_nonzero(m) : bytes_bit(c, 1), d);
        return;
    }
    const uint32_t kept = bytes_nonzero(m), marker = bytes_bit(c, 1), thresh = bytes_bit(c, 0);
    // the three colours' channels: B only where dropped, G where kept and no marker, R wherever kept; all 0 where the frame shows
    const uint32_t blue = thresh & ~kept, green = kept & ~marker, red = kept;
    uint32_t painted[3];
    thrice(kept | thresh, painted);
    d[0] = (fr[0] & ~painted[0]) | perm(red, perm(green, blue, 0x01000400u), 0x03040100u);      // B0 G0 R0 B1
    d[1] = (fr[1] & ~painted[1]) | perm(red, perm(green, blue, 0x06020005u), 0x03020500u);      // G1 R1 B2 G2
    d[2] = (fr[2] & ~painted[2]) | perm(red, perm(green, blue, 0x00070300u), 0x07020106u);      // R2 B3 G3 R3
}

// Sixteen pixels: 16 bytes at cls and at mask, 16 * channels at frame (read as the mode needs them), 48 bytes to dst.  No
// pointer needs any alignment.
YSMR_HD_FORCE void step16(int mode, int channels, const uint8_t *frame, const uint8_t *cls, const uint8_t *mask, uint8_t *dst)
{
    uint32_t c[4] = {0, 0, 0, 0}, m[4] = {0, 0, 0, 0}, fr[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, d[12];
    if (mode != MODE_MARKERS) __builtin_memcpy(m, mask, 16);
    if (mode != MODE_MASK) __builtin_memcpy(c, cls, 16);
    if (mode == MODE_CLASSES) {
        if (channels == 3) {
            __builtin_memcpy(fr, frame, 48);
        } else {
            uint32_t g[4];
            __builtin_memcpy(g, frame, 16);
            for (int q = 0; q < 4; ++q) thrice(g[q], fr + 3 * q);
        }
    }
    for (int q = 0; q < 4; ++q) quad(mode, c[q], m[q], fr + 3 * q, d + 3 * q);
    __builtin_memcpy(dst, d, 48);
}

// A stored row of W pixels: steps of 16 from pixel `begin` on, `stride16` pixels apart (the device: lane * 16 and 64 * 16; the
// host: 0 and 16), and behind them, for lane < W % 16, a pixel of the tail.  cls, mask, frame: the row's first bytes.
YSMR_HD_FORCE void row(int mode, int channels, const uint8_t *frame, const uint8_t *cls, const uint8_t *mask, int W, int begin, int stride16,
                       int lane, uint8_t *dst)
{
    const int whole = W & ~15;
    for (int x = begin; x < whole; x += stride16)      // (a pointer the mode does not read may be NULL: nothing is added to it)
        step16(mode, channels, mode == MODE_CLASSES ? frame + (size_t)x * channels : frame, cls + x, mode == MODE_MARKERS ? mask : mask + x,
               dst + 3 * (size_t)x);
    if (whole + lane < W) {
        const int x = whole + lane;
        uint8_t b = 0, g = 0, r = 0;
        if (mode == MODE_CLASSES) {
            const uint8_t *src = frame + (size_t)x * channels;
            b = src[0]; g = src[channels == 3 ? 1 : 0]; r = src[channels == 3 ? 2 : 0];
        }
        pixel(mode, mode == MODE_MASK ? 0u : cls[x], mode == MODE_MARKERS ? 0u : mask[x], b, g, r, dst + 3 * (size_t)x);
    }
}

// The arguments both entries check: NULL, or what is wrong with them.  (frames: needed in mode 2 only; mask: not in mode 1.)
inline const char *check_args(const void *frames, const void *cls, const void *mask, int n_frames, int H, int W, int channels, int mode,
                              const void *out, int stride, size_t frame_bytes)
{
    if (mode != MODE_MASK && mode != MODE_MARKERS && mode != MODE_CLASSES) return "mode must be 0 (mask), 1 (markers) or 2 (classes)";
    if (channels != 1 && channels != 3) return "channels must be 1 or 3";
    if (!cls) return "cls must not be NULL";
    if (!mask && mode != MODE_MARKERS) return "mask must not be NULL in modes 0 and 2";
    if (!frames && mode == MODE_CLASSES) return "frames must not be NULL in mode 2";
    return view::check_layout(n_frames, H, W, stride, frame_bytes, out);
}

// The view of a batch on host arrays.  NULL, or the reason why nothing was done.
inline const char *batch_host(const uint8_t *frames, const uint8_t *cls, const uint8_t *mask, int n_frames, int H, int W, int channels,
                              int mode, uint8_t *out, int stride, size_t frame_bytes, int bottom_up)
{
    if (const char *why = check_args(frames, cls, mask, n_frames, H, W, channels, mode, out, stride, frame_bytes)) return why;
    for (int f = 0; f < n_frames; ++f)
        for (int y = 0; y < H; ++y) {
            const size_t first = ((size_t)f * H + y) * (size_t)W;
            uint8_t *dst = view::dib_row(out + (size_t)f * frame_bytes, H, stride, bottom_up, y);
            // (pointers that are NULL in this mode stay NULL: nothing is added to them and nothing reads them)
            const uint8_t *fr = mode == MODE_CLASSES ? frames + first * (size_t)channels : nullptr;
            const uint8_t *mk = mode == MODE_MARKERS ? nullptr : mask + first;
            row(mode, channels, fr, cls + first, mk, W, 0, 16, 0, dst);
            for (int lane = 1; lane < (W & 15); ++lane) row(mode, channels, fr, cls + first, mk, W, W, 16, lane, dst);   // (the tail's other pixels)
            for (size_t k = (size_t)W * 3; k < (size_t)stride; ++k) dst[k] = 0;
        }
    return nullptr;
}

}  // namespace thrview
}  // namespace ysmr
