// glyph.h -- the lettering of a track's mark, shared by annotate.hip (the annotated video) and view.hip (the detection
// view): the 5 x 7 digits, where the digits of an id and the dot sit relative to the mark's (x, y), and which pixels they
// are.  Plain C++ as well as HIP (the host twin of the detection view and a stand-alone host program compile it alone).
#pragma once
#include <cstdint>
#include "hd.h"
#include "ysmr_hip.h"

namespace ysmr {
namespace glyph {

constexpr int GLYPH_W = 5, GLYPH_H = 7, GLYPH_STEP = 6;   // a digit cell: 5 x 7 pixels, the next digit starts 6 to the right
constexpr int TEXT_DX = -10, TEXT_DY = -16;               // top-left pixel of the first digit, from the mark's (x, y)
constexpr int MAX_PIXELS = 10 * GLYPH_W * GLYPH_H + 5;    // ten digits and a large dot

// 5 x 7 digits, rows top to bottom, five bits each, most significant = left column; row r sits in bits [30 - 5r, 34 - 5r]
#define YSMR_GLYPH(a, b, c, d, e, f, g)                                                                                     \
    (((uint64_t)0b##a << 30) | ((uint64_t)0b##b << 25) | ((uint64_t)0b##c << 20) | ((uint64_t)0b##d << 15) |                \
     ((uint64_t)0b##e << 10) | ((uint64_t)0b##f << 5) | (uint64_t)0b##g)
#define YSMR_GLYPH_TABLE                                                                                                    \
    {YSMR_GLYPH(01110, 10001, 10011, 10101, 11001, 10001, 01110), YSMR_GLYPH(00100, 01100, 00100, 00100, 00100, 00100, 01110), \
     YSMR_GLYPH(01110, 10001, 00001, 00010, 00100, 01000, 11111), YSMR_GLYPH(11111, 00010, 00100, 00010, 00001, 10001, 01110), \
     YSMR_GLYPH(00010, 00110, 01010, 10010, 11111, 00010, 00010), YSMR_GLYPH(11111, 10000, 11110, 00001, 00001, 10001, 01110), \
     YSMR_GLYPH(00110, 01000, 10000, 11110, 10001, 10001, 01110), YSMR_GLYPH(11111, 00001, 00010, 00100, 01000, 01000, 01000), \
     YSMR_GLYPH(01110, 10001, 10001, 01110, 10001, 10001, 01110), YSMR_GLYPH(01110, 10001, 10001, 01111, 00001, 00010, 01100)}
// (one table, held twice: device code reads it from constant memory, host code from a constexpr array)
#ifdef __HIPCC__
static __constant__ uint64_t c_glyph[10] = YSMR_GLYPH_TABLE;
#endif
constexpr uint64_t h_glyph[10] = YSMR_GLYPH_TABLE;
#undef YSMR_GLYPH_TABLE
#undef YSMR_GLYPH

YSMR_HD_FORCE uint64_t glyph_bits(unsigned digit)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return c_glyph[digit];
#else
    return h_glyph[digit];
#endif
}

// What a painter needs to know of a mark: where its digits are and which, and how large its dot is.
struct Mark {
    long long x, y;       // 64 bits: a coordinate anywhere in int32 stays exact through the offsets below
    uint64_t digits;      // four bits per decimal digit of the id, the leading one in bits [0, 4)
    int nd, big;          // number of digits (1 .. 10); dot of radius 1 (style 2)
};

YSMR_HD_FORCE Mark mark_of(const ysmr_mark &m)
{
    Mark r;
    r.x = m.x; r.y = m.y; r.big = m.style == 2u;
    uint32_t v = m.track_id;
    r.digits = 0; r.nd = 0;
    do { r.digits = (r.digits << 4) | (v % 10u); v /= 10u; ++r.nd; } while (v);      // least significant digit in last
    return r;
}

// How many pixel cells a mark has: 35 per digit, then the dot's one or five.
YSMR_HD_FORCE int mark_cells(const Mark &m) { return m.nd * GLYPH_W * GLYPH_H + (m.big ? 5 : 1); }

// Cell p of a mark: where it is, and whether it is painted (false, and px / py untouched, for p >= mark_cells).  Digit k, row r,
// column c lands on (x - 10 + 6k + c, y - 16 + r); the dot is (x, y), for the larger one also its four edge neighbours.
YSMR_HD_FORCE bool mark_cell(const Mark &m, int p, long long &px, long long &py)
{
    const int cells = m.nd * GLYPH_W * GLYPH_H, total = cells + (m.big ? 5 : 1);
    bool on = false;
    if (p < cells) {
        const int k = p / (GLYPH_W * GLYPH_H), q = p - k * (GLYPH_W * GLYPH_H), row = q / GLYPH_W, c = q - row * GLYPH_W;
        px = m.x + TEXT_DX + GLYPH_STEP * k + c;
        py = m.y + TEXT_DY + row;
        on = (glyph_bits((unsigned)(m.digits >> (4 * k)) & 15u) >> (34 - q)) & 1u;
    } else if (p < total) {
        const int d = p - cells;                                   // 0: the centre; 1 .. 4: left, right, up, down
        px = m.x + (d == 1 ? -1 : d == 2 ? 1 : 0);
        py = m.y + (d == 3 ? -1 : d == 4 ? 1 : 0);
        on = true;
    }
    return on;
}

// Does `m` paint the pixel (px, py)?
YSMR_HD_FORCE bool covers(const Mark &m, long long px, long long py)
{
    const long long ax = px > m.x ? px - m.x : m.x - px, ay = py > m.y ? py - m.y : m.y - py;
    if (ax + ay <= (long long)m.big) return true;
    const long long dx = px - (m.x + TEXT_DX), dy = py - (m.y + TEXT_DY);
    if (dx < 0 || dy < 0 || dy >= GLYPH_H || dx >= (long long)GLYPH_STEP * m.nd) return false;
    const int k = (int)dx / GLYPH_STEP, c = (int)dx - k * GLYPH_STEP;
    if (c >= GLYPH_W) return false;
    const uint64_t g = glyph_bits((unsigned)(m.digits >> (4 * k)) & 15u);
    return (g >> (34 - (GLYPH_W * (int)dy + c))) & 1u;
}

}  // namespace glyph
}  // namespace ysmr
