// view_rule.h -- which pixels the detection view paints, in the one form that the kernels of view.hip, their host twin
// ysmr_view_batch_host and a stand-alone host program all compile (plain C++ as well as HIP).
//
// PIXEL RULE.  A frame is expanded to B, G, R (gray: B = G = R) and stored as a DIB frame; then two layers, later over earlier:
//   1. boxes   for every detection the closed outline of np.intp(cv2.boxPoints(rect)) (quad.h: the corners ysmr_luminosity_batch
//              computes): the four 8-connected lines corner i-1 -> corner i, walked left to right, pixels outside the frame
//              dropped, nothing clipped beforehand; colour (255, 0, 0).  A box whose corners coincide paints its pixel.
//   2. tracks  for every row the link emitted for the frame, the id's decimal digits and the single-pixel dot at (int(x),
//              int(y)), truncated toward zero: style 0 of ysmr_annotate_batch (glyph.h); colour (0, 255, 0).
// Inside a layer every mark has one colour, so no order among them can show.  Integers only once the corners are known.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include "glyph.h"
#include "hd.h"
#include "quad.h"
#include "ysmr_hip.h"

namespace ysmr {
namespace view {

// the stored row of pixel row y
YSMR_HD_FORCE uint8_t *dib_row(uint8_t *frame, int H, int stride, int bottom_up, int y)
{
    return frame + (size_t)(bottom_up ? H - 1 - y : y) * (size_t)stride;
}

// Edge i (corner i-1 -> corner i) of the box of one detection q = (cx, cy, w, h, angle).  (No indexing by i: on the device the
// corners stay in registers.)
YSMR_HD_FORCE void edge_of(const float *q, int i, LumEdge &e)
{
    const double rad = lum_radians(q[4]);
    int px[4], py[4];
    lum_corners(q[0], q[1], q[2], q[3], (float)cos(rad), (float)sin(rad), px, py);
    const int ax = i == 0 ? px[3] : i == 1 ? px[0] : i == 2 ? px[1] : px[2], ay = i == 0 ? py[3] : i == 1 ? py[0] : i == 2 ? py[1] : py[2];
    const int bx = i == 0 ? px[0] : i == 1 ? px[1] : i == 2 ? px[2] : px[3], by = i == 0 ? py[0] : i == 1 ? py[1] : i == 2 ? py[2] : py[3];
    lum_edge_make(ax, ay, bx, by, e);
}

// The rows of the frame that an edge's line touches: [first, last], empty if first > last.
YSMR_HD_FORCE void edge_rows(const LumEdge &e, int H, int &first, int &last)
{
    const int y1 = e.y0 + e.sy * e.ady;
    first = lum_max(lum_min(e.y0, y1), 0);
    last = lum_min(lum_max(e.y0, y1), H - 1);
}

// The edge's pixels on row y (0 <= y < H) into the stored row: one run, cut to [0, W) -- at most W stores, wherever the
// corners are.
YSMR_HD_FORCE void outline_row(const LumEdge &e, int y, int W, uint8_t *row)
{
    int a, b;
    if (!lum_edge_row(e, y, a, b)) return;
    a = lum_max(a, 0); b = lum_min(b, W - 1);
    for (int x = a; x <= b; ++x) {
        uint8_t *p = row + 3 * (size_t)x;
        p[0] = 255; p[1] = 0; p[2] = 0;
    }
}

// The mark of a row in a batch that begins at frame `first`: false for a row of another batch, or one whose position is not
// finite.  Positions beyond int32 are moved to its ends (far outside any frame either way).
YSMR_HD_FORCE bool mark_of_row(const ysmr_row &r, int first, int n_frames, int &f, glyph::Mark &m)
{
    const long long rel = (long long)r.frame - first;
    if (rel < 0 || rel >= n_frames) return false;
    if (!(r.x == r.x) || !(r.y == r.y) || fabs(r.x) > 1.7e308 || fabs(r.y) > 1.7e308) return false;
    f = (int)rel;
    const double lo = -2147483648.0, hi = 2147483647.0;
    ysmr_mark k;
    k.x = (int32_t)(r.x < lo ? lo : r.x > hi ? hi : r.x);      // (a conversion truncates toward zero, as int())
    k.y = (int32_t)(r.y < lo ? lo : r.y > hi ? hi : r.y);
    k.track_id = (uint32_t)r.track_id;
    k.style = 0;
    m = glyph::mark_of(k);
    return true;
}

// Cell p of a mark into the stored frame, if it is painted and inside.
YSMR_HD_FORCE void paint_cell(const glyph::Mark &m, int p, int H, int W, int stride, int bottom_up, uint8_t *frame)
{
    long long px = -1, py = -1;
    if (!glyph::mark_cell(m, p, px, py) || px < 0 || px >= W || py < 0 || py >= H) return;
    uint8_t *q = dib_row(frame, H, stride, bottom_up, (int)py) + 3 * (size_t)px;
    q[0] = 0; q[1] = 255; q[2] = 0;
}

// The arguments every entry checks: NULL, or what is wrong with them.
inline const char *check_layout(int n_frames, int H, int W, int stride, size_t frame_bytes, const void *dib)
{
    if (n_frames <= 0 || H <= 0 || W <= 0) return "n_frames, height, width must be positive";
    if ((long long)stride < 3LL * W || (stride & 3) || frame_bytes < (size_t)stride * (size_t)H) return "stride (a multiple of 4) / frame_bytes too small for the frame";
    if (!dib) return "the DIB buffer must not be NULL";
    if (((uintptr_t)dib & 3) || (frame_bytes & 3)) return "the DIB buffer and frame_bytes must be 4-byte aligned";
    return nullptr;
}

// The whole view of a batch on host arrays: pack (as ysmr_annotate_batch without marks), boxes, tracks.  NULL, or the reason
// why nothing was done.  rows may be NULL when row_begin >= row_end.
inline const char *batch_host(const uint8_t *frames, int n_frames, int H, int W, int channels, const float *det,
                              const int32_t *det_count, int max_det, const ysmr_row *rows, long long row_begin, long long row_end,
                              int first_frame_index, uint8_t *out, int stride, size_t frame_bytes, int bottom_up)
{
    if (const char *why = check_layout(n_frames, H, W, stride, frame_bytes, out)) return why;
    if (channels != 1 && channels != 3) return "channels must be 1 or 3";
    if (!frames || !det || !det_count || max_det <= 0) return "frames, det, det_count must not be NULL and max_det positive";
    if (row_begin < row_end && !rows) return "rows must not be NULL when there are rows";
    for (int f = 0; f < n_frames; ++f) {
        uint8_t *frame = out + (size_t)f * frame_bytes;
        for (int y = 0; y < H; ++y) {
            const uint8_t *src = frames + ((size_t)f * H + y) * (size_t)W * channels;
            uint8_t *dst = dib_row(frame, H, stride, bottom_up, y);
            if (channels == 3) memcpy(dst, src, (size_t)W * 3);
            else for (int x = 0; x < W; ++x) dst[3 * x] = dst[3 * x + 1] = dst[3 * x + 2] = src[x];
            memset(dst + (size_t)W * 3, 0, (size_t)stride - (size_t)W * 3);
        }
        const int n = lum_min(lum_max(det_count[f], 0), max_det);
        for (int d = 0; d < n; ++d)
            for (int i = 0; i < 4; ++i) {
                LumEdge e;
                int first, last;
                edge_of(det + ((size_t)f * max_det + d) * 5, i, e);
                edge_rows(e, H, first, last);
                for (int y = first; y <= last; ++y) outline_row(e, y, W, dib_row(frame, H, stride, bottom_up, y));
            }
    }
    for (long long i = row_begin; i < row_end; ++i) {
        int f;
        glyph::Mark m;
        if (!mark_of_row(rows[i], first_frame_index, n_frames, f, m)) continue;
        for (int p = 0, total = glyph::mark_cells(m); p < total; ++p) paint_cell(m, p, H, W, stride, bottom_up, out + (size_t)f * frame_bytes);
    }
    return nullptr;
}

}  // namespace view
}  // namespace ysmr
