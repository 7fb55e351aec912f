// annotate.hip -- the frames of the annotated output video (ysmr/track_eval.py:1321-1472): what cv2.putText, cv2.circle and
// cv2.VideoWriter.write do to a frame between cap.read() and the file, for an uncompressed 24-bit stream.  ingest.hip's byte
// work in the other direction: device-resident frames become stored DIB frames (B, G, R per pixel, rows padded to 4 bytes,
// bottom-up on request), with the marks of the tracks painted on the way.  Two launches on the caller's stream:
//   k_pack_dib    every byte of every output frame, padding included, from the frame as it was read;
//   k_paint_marks the marks on top of that.
// PAINT RULE.  A sequential painter goes frame by frame, mark by mark in table order, text first and then the dot, later
// paint over earlier, pixels outside the frame dropped.  Here a wave takes one mark and a lane one of its pixels, and a
// pixel is stored only if NO LATER MARK OF THE SAME FRAME COVERS IT: of all the marks that cover an output pixel exactly one
// -- the last in table order -- stores it, once (a mark's text and its dot cannot meet: the text ends six rows above the
// dot's top), and it stores what the sequential painter leaves there.  No two lanes of the launch write the same byte, so
// the result does not depend on scheduling; no atomics, no owner map.
#include "common.h"
#include "glyph.h"
#include <algorithm>

namespace {

using namespace ysmr::glyph;   // the digits and where a mark's pixels are: shared with view.hip

constexpr int PACK_BLOCKS = 1024;    // resident grids (see ingest.hip)
constexpr int PAINT_BLOCKS = 1024;
__device__ __forceinline__ uint4 ld16(const uint8_t *p) { uint4 v; __builtin_memcpy(&v, p, 16); return v; }
__device__ __forceinline__ void st16(uint8_t *p, const uint4 &v) { __builtin_memcpy(p, &v, 16); }

// A WAVE writes one stored row at a time (k_unpack_dib's shape: one division per 64 lanes, 16 bytes per lane and access,
// neither end aligned beyond the 4 bytes of a DIB row).  BGR rows are copied; of a gray row a lane reads 16 pixels and
// writes their 48 bytes; what is left of the row goes pixel by pixel, and the padding bytes are zeroed.
template <int CH>
__global__ __launch_bounds__(256) void k_pack_dib(const uint8_t *__restrict__ frames, int n, int H, int W, int bottom_up,
                                                  uint8_t *__restrict__ out, int out_stride, size_t out_frame_bytes)
{
    const int lane = threadIdx.x & 63;
    const long long rows = (long long)n * H, wave0 = (long long)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (long long)gridDim.x * 4;
    const size_t row_bytes = (size_t)W * 3;
    for (long long item = wave0; item < rows; item += nwaves) {
        const long long f = item / H;
        const int y = (int)(item - f * H);
        const uint8_t *src = frames + (size_t)item * W * CH;
        uint8_t *dst = out + (size_t)f * out_frame_bytes + (size_t)(bottom_up ? H - 1 - y : y) * out_stride;
        if (CH == 3) {
            const size_t whole = row_bytes & ~(size_t)15;
            for (size_t b = (size_t)lane * 16; b < whole; b += 64 * 16) st16(dst + b, ld16(src + b));
            if (whole + lane < row_bytes) dst[whole + lane] = src[whole + lane];
        } else {
            const int whole = W & ~15;
            for (int x = lane * 16; x < whole; x += 64 * 16) {
                uint8_t g[16], o[48];
                __builtin_memcpy(g, src + x, 16);
#pragma unroll
                for (int k = 0; k < 16; ++k) o[3 * k] = o[3 * k + 1] = o[3 * k + 2] = g[k];
                __builtin_memcpy(dst + 3 * (size_t)x, o, 48);
            }
            if (whole + lane < W) {
                const uint8_t g = src[whole + lane];
                uint8_t *p = dst + 3 * (size_t)(whole + lane);
                p[0] = g; p[1] = g; p[2] = g;
            }
        }
        for (size_t b = row_bytes + lane; b < (size_t)out_stride; b += 64) dst[b] = 0;   // (three bytes at most in a DIB)
    }
}

// A WAVE paints one mark at a time; its pixels -- 35 cells per digit, then the dot's one or five -- are dealt to the lanes
// 64 at a time (six rounds at most: ten digits and a large dot are 355).  A lane keeps one bit per round: "this pixel is
// mine, inside the frame, and still visible".  The later marks of the frame are then read 64 at a time, a lane each, and
// tested box against box; the few whose boxes meet this mark's are gone through one by one, every lane clearing the bits of
// the pixels that mark paints.  What is left is stored.
constexpr int MAX_ROUNDS = (MAX_PIXELS + 63) / 64;

__global__ __launch_bounds__(256) void k_paint_marks(const ysmr_mark *__restrict__ marks, const long long *__restrict__ first,
                                                     int n, int H, int W, int bottom_up, uint8_t *__restrict__ out, int out_stride,
                                                     size_t out_frame_bytes)
{
    const int lane = threadIdx.x & 63;
    const long long begin = first[0], end = first[n];
    const long long wave0 = (long long)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (long long)gridDim.x * 4;
    for (long long item = begin + wave0; item < end; item += nwaves) {
        // the frame of this mark: the last f with first[f] <= item (frames without marks repeat a value)
        int lo = 0, hi = n;
        while (hi - lo > 1) {
            const int mid = lo + (hi - lo) / 2;
            if (first[mid] <= item) lo = mid; else hi = mid;
        }
        const int f = lo;
        const long long frame_end = std::min(first[f + 1], end);
        const ysmr_mark raw = marks[item];
        const Mark me = mark_of(raw);

        // my pixels
        long long px[MAX_ROUNDS], py[MAX_ROUNDS];
        uint32_t alive = 0;
#pragma unroll
        for (int r = 0; r < MAX_ROUNDS; ++r) {
            px[r] = py[r] = -1;
            const bool on = mark_cell(me, r * 64 + lane, px[r], py[r]);
            if (on && px[r] >= 0 && px[r] < W && py[r] >= 0 && py[r] < H) alive |= 1u << r;
        }

        // later marks of this frame that may paint over them: box test per lane, exact test for the boxes that meet.
        // (A mark's box: its text, x - 10 .. x - 10 + 6 nd - 2 by y - 16 .. y - 10, joined with its dot: x - 10 .. the larger
        // of x + 1 and the text's right end, y - 16 .. y + 1.)
        const long long my_x0 = me.x + TEXT_DX, my_x1 = std::max(me.x + 1, me.x + TEXT_DX + (long long)GLYPH_STEP * me.nd - 2);
        const long long my_y0 = me.y + TEXT_DY, my_y1 = me.y + 1;
        for (long long base = item + 1; base < frame_end; base += 64) {
            bool meets = false;
            if (base + lane < frame_end) {
                const ysmr_mark o = marks[base + lane];
                int nd = 1;
                for (uint32_t v = o.track_id; v >= 10u; v /= 10u) ++nd;
                const long long ox = o.x, oy = o.y;
                const long long x0 = ox + TEXT_DX, x1 = std::max(ox + 1, ox + TEXT_DX + (long long)GLYPH_STEP * nd - 2);
                meets = x0 <= my_x1 && my_x0 <= x1 && oy + TEXT_DY <= my_y1 && my_y0 <= oy + 1;
            }
            unsigned long long hits = __ballot(meets);
            while (hits) {
                const int j = __ffsll(hits) - 1;
                hits &= hits - 1;
                const Mark other = mark_of(marks[base + j]);               // (the same address in every lane)
#pragma unroll
                for (int r = 0; r < MAX_ROUNDS; ++r)
                    if ((alive >> r & 1u) && covers(other, px[r], py[r])) alive &= ~(1u << r);
            }
        }

        const uint8_t cb = raw.style == 1u ? 15 : raw.style == 2u ? 255 : 0;
        const uint8_t cg = raw.style == 1u ? 165 : 255;
        const uint8_t cr = raw.style == 1u ? 253 : raw.style == 2u ? 255 : 0;
        uint8_t *frame = out + (size_t)f * out_frame_bytes;
#pragma unroll
        for (int r = 0; r < MAX_ROUNDS; ++r)
            if (alive >> r & 1u) {
                uint8_t *p = frame + (size_t)(bottom_up ? H - 1 - py[r] : py[r]) * out_stride + 3 * (size_t)px[r];
                p[0] = cb; p[1] = cg; p[2] = cr;
            }
    }
}

}  // namespace

extern "C" int ysmr_annotate_batch(void *stream, const uint8_t *frames_dev, int n_frames, int height, int width, int channels,
                                   const ysmr_mark *marks_dev, const int64_t *first_dev, uint8_t *out_dev, int out_stride,
                                   size_t out_frame_bytes, int bottom_up)
{
    if (n_frames <= 0 || height <= 0 || width <= 0)
        return ysmr::fail(YSMR_ERR_ARG, "n_frames, height, width must be positive (got %d, %d, %d)", n_frames, height, width);
    if (channels != 1 && channels != 3) return ysmr::fail(YSMR_ERR_ARG, "channels must be 1 or 3, got %d", channels);
    if ((long long)out_stride < 3LL * width || (out_stride & 3) || out_frame_bytes < (size_t)out_stride * height)
        return ysmr::fail(YSMR_ERR_ARG, "out_stride %d (a multiple of 4) / out_frame_bytes %zu too small for %d x %d x 3", out_stride,
                          out_frame_bytes, width, height);
    if (!frames_dev || !out_dev) return ysmr::fail(YSMR_ERR_ARG, "frames_dev and out_dev must not be NULL");
    if (first_dev && !marks_dev) return ysmr::fail(YSMR_ERR_ARG, "marks_dev must not be NULL when first_dev is given");
    if (((uintptr_t)out_dev & 3) || (out_frame_bytes & 3)) return ysmr::fail(YSMR_ERR_ARG, "out_dev and out_frame_bytes must be 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const size_t blocks = std::min<size_t>(((size_t)n_frames * height + 3) / 4, PACK_BLOCKS);   // four rows (waves) per block
    if (channels == 3)
        hipLaunchKernelGGL(k_pack_dib<3>, dim3((unsigned)blocks), dim3(256), 0, st, frames_dev, n_frames, height, width, bottom_up,
                           out_dev, out_stride, out_frame_bytes);
    else
        hipLaunchKernelGGL(k_pack_dib<1>, dim3((unsigned)blocks), dim3(256), 0, st, frames_dev, n_frames, height, width, bottom_up,
                           out_dev, out_stride, out_frame_bytes);
    YSMR_LAUNCH_CHECK();
    if (first_dev) {   // (how many marks there are is on the device: a resident grid goes through them)
        hipLaunchKernelGGL(k_paint_marks, dim3(PAINT_BLOCKS), dim3(256), 0, st, marks_dev, (const long long *)first_dev, n_frames,
                           height, width, bottom_up, out_dev, out_stride, out_frame_bytes);
        YSMR_LAUNCH_CHECK();
    }
    return YSMR_OK;
}
