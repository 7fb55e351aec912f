// quad.h -- np.intp(cv2.boxPoints(rect)) of a detection and the pixels of its four edge lines, shared by luminosity.hip (the
// filled box: mean gray value under it) and view.hip (its outline in the detection view).  Plain C++ as well as HIP: the
// host twins of both and a stand-alone host program compile it alone.
//
// An edge's pixels on row y come in closed form instead of by walking the line: the 8-connected LineIterator's error term
// after i major steps is ((d_major - 2 d_minor i) mod 2 d_major) - 2 d_minor, hence its minor steps so far are
// floor((2 d_minor i + d_major - 1) / (2 d_major)); inverted, that gives the x-run of an x-major line on a row and the one
// pixel of a y-major line.  The work per row does not depend on where the corners are.
#pragma once
#include <cmath>
#include <cstdint>
#include "hd.h"

constexpr float LUM_CLAMP = 1048576.0f;              // corners beyond +-2^20 are moved there (no frame is that large)

struct LumEdge {
    // the edge as LineIterator(leftToRight) walks it ...
    int x0, y0, dx, ady, sy;
    // ... and as the scanline fill's edge table holds it (horizontal edges: yt == yb, never active)
    int yt, yb;
    long long xt16, dxs;
};

struct LumBox { int px[4], py[4]; LumEdge e[4]; int ymin, ymax; };

YSMR_HD_FORCE int lum_min(int a, int b) { return a < b ? a : b; }
YSMR_HD_FORCE int lum_max(int a, int b) { return a > b ? a : b; }

// floor(num / den) for 0 <= num < 2^52, 0 < den < 2^31: a float64 quotient is off by at most one
YSMR_HD_FORCE long long lum_floor_div(long long num, long long den)
{
    long long q = (long long)((double)num / (double)den);
    if (q * den > num) --q;
    else if ((q + 1) * den <= num) ++q;
    return q;
}

YSMR_HD_FORCE int lum_trunc(float v)
{
    return (int)fminf(fmaxf(v, -LUM_CLAMP), LUM_CLAMP);     // (a NaN ends at -2^20)
}

YSMR_HD_FORCE double lum_radians(float angle) { return (double)angle * 3.14159265358979323846 / 180.0; }

// np.intp(cv2.boxPoints(rect)): the four corners.  c / s: cos and sin of the angle, already float32.
YSMR_HD_FORCE void lum_corners(float cx, float cy, float w, float h, float c, float s, int px[4], int py[4])
{
    const float b = c * 0.5f, a = s * 0.5f;
    const float p0x = cx - a * h - b * w, p0y = cy + b * h - a * w;
    const float p1x = cx + a * h - b * w, p1y = cy - b * h - a * w;
    px[0] = lum_trunc(p0x); py[0] = lum_trunc(p0y);
    px[1] = lum_trunc(p1x); py[1] = lum_trunc(p1y);
    px[2] = lum_trunc(2.0f * cx - p0x); py[2] = lum_trunc(2.0f * cy - p0y);
    px[3] = lum_trunc(2.0f * cx - p1x); py[3] = lum_trunc(2.0f * cy - p1y);
}

// The tables of the edge (ax, ay) -> (bx, by).
YSMR_HD_FORCE void lum_edge_make(int ax, int ay, int bx, int by, LumEdge &e)
{
    const bool swap = bx < ax;
    e.x0 = swap ? bx : ax; e.y0 = swap ? by : ay;
    const int x1 = swap ? ax : bx, y1 = swap ? ay : by;
    e.dx = x1 - e.x0;
    e.sy = y1 >= e.y0 ? 1 : -1;
    e.ady = (y1 - e.y0) * e.sy;
    const bool down = ay < by;
    e.yt = down ? ay : by; e.yb = down ? by : ay;
    const int xt = down ? ax : bx, xb = down ? bx : ax;
    e.xt16 = (long long)xt * 65536;                 // (16.16; a product, not a shift: xt may be negative)
    e.dxs = 0;
    if (e.yb > e.yt) {                              // C division truncates toward zero
        const long long d = ((long long)xb - xt) * 65536;
        const long long q = lum_floor_div(d < 0 ? -d : d, e.yb - e.yt);
        e.dxs = d < 0 ? -q : q;
    }
}

// The corners and the tables of the four edges pts[i - 1] -> pts[i].
YSMR_HD_FORCE void lum_box(float cx, float cy, float w, float h, float c, float s, LumBox &B)
{
    lum_corners(cx, cy, w, h, c, s, B.px, B.py);
    B.ymin = lum_min(lum_min(B.py[0], B.py[1]), lum_min(B.py[2], B.py[3]));
    B.ymax = lum_max(lum_max(B.py[0], B.py[1]), lum_max(B.py[2], B.py[3]));
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int j = (i + 3) & 3;
        lum_edge_make(B.px[j], B.py[j], B.px[i], B.py[i], B.e[i]);
    }
}

// The pixels [a, b] of the edge's 8-connected line on row y, not clipped: false when the line has none there.
YSMR_HD_FORCE bool lum_edge_row(const LumEdge &e, int y, int &a, int &b)
{
    const int k = (y - e.y0) * e.sy;
    if (k < 0 || k > e.ady) return false;
    if (e.ady > e.dx) {                                 // y-major: one pixel per row
        a = b = e.x0 + (int)lum_floor_div(2ll * e.dx * k + e.ady - 1, 2ll * e.ady);
    } else if (e.ady == 0) {
        a = e.x0; b = e.x0 + e.dx;
    } else {                                            // x-major: the major steps whose minor count is k
        const long long num = 2ll * e.dx * k - e.dx + 2ll * e.ady;
        const int i_lo = num < 0 ? 0 : (int)lum_floor_div(num, 2ll * e.ady);
        const long long i_hi = lum_floor_div(2ll * e.dx * k + e.dx, 2ll * e.ady);
        a = e.x0 + i_lo; b = e.x0 + (int)(i_hi < (long long)e.dx ? i_hi : (long long)e.dx);
    }
    return true;
}
